"""Every consumer of the fixed-base window tables (dapol_amd/csrc/tables.h) at the window widths that matter, fed with scalars that
sit on the edges of the signed-digit recoding (tests/edge_scalars.py): commitments, padding nodes, tree build / update / remove, the
prover with steered nonces in both digit layouts, seed-mode proving, the verifier's two paths and the policy provers.  Bit-exact
against the oracles, which tests/test_edge_scalars_cpu.py has checked against each other on the same crafted tapes.

A context picks its width from the memory that happens to be free (dapol_ctx_create), so the contexts here pin theirs through
dapol_options.window_bits; one context lives at a time and none holds more than about 20 GB of tables:
    W <= 17: 8 parties, once with the high-half rows forced on and once forced off (17.4 GB / 8.8 GB at W = 17)
    W = 20:  2 parties without high-half rows (18.9 GB)
Every test runs under a time limit of its own: a step that hangs ends the process instead of holding the card."""
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest

import edge_scalars as E
from conftest import load_golden
import test_gpu_parity as parity
from test_gpu_parity import SEED, _arr, _rand_leaves, _ref_root, _ref_tree

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 240          # per test; the slowest takes seconds
CTX_LIMIT_S = 240           # per context creation (the tables of the widest are 19 GB)


def _parties(W):
    return 8 if W <= 17 else 2


CONTEXTS = [(W, hi, _parties(W)) for W in E.WIDTHS for hi in ((+1, -1) if W <= 17 else (-1,))]


def _ctx_id(c):
    return "W%d-%s-P%d" % (c[0], "hi" if c[1] > 0 else "nohi", c[2])


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


def _make_ctx(hip_lib, W, hi, P):
    faulthandler.dump_traceback_later(CTX_LIMIT_S, exit=True, file=sys.__stderr__)
    try:
        ctx = hip_lib.Context(0, P, options=hip_lib.Options(window_bits=W, high_half_rows=hi))
    finally:
        faulthandler.cancel_dump_traceback_later()
    o = ctx.get_options()
    assert (o.window_bits, o.high_half_rows) == (W, hi)
    return ctx


@pytest.fixture(scope="module", params=CONTEXTS, ids=_ctx_id)
def wc(request, hip_lib):
    """(W, high_half_rows, max_parties, context): pytest runs all the tests of one context before it makes the next."""
    W, hi, P = request.param
    ctx = _make_ctx(hip_lib, W, hi, P)
    yield W, hi, P, ctx
    ctx.close()


_cache = {}                 # oracle results that do not depend on the context (only on the width, or on nothing)


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bytes32(xs):
    return np.array([list(E.le32(x)) for x in xs], np.uint8).reshape(len(xs), 32)


def _canon(W):
    f = E.families(W, "canonical")
    return [f[k] for k in sorted(f)]


def _blind(W):
    """The blinding families (several of them >= l: Scalar::from_bits inputs) and the canonical ones, whose carry chains end lower."""
    f = E.families(W, "blinding")
    c = E.families(W, "canonical")
    return [f[k] for k in sorted(f)] + [c[k] for k in ("allneg", "allpos", "althalf")]


def _values(W):
    f = E.families(W, "value")
    return [f[k] for k in sorted(f)]


# ---------------------------------------------------------------------------------------------------- C.1 golden files
def test_golden_files(wc, hip_lib):
    """commit.json, trees.json (root, every level, paths), range.json and dapol.json as tests/test_gpu_parity.py runs them on the
    default context; the proof shapes with more parties than the context holds are left to the contexts that hold them."""
    W, hi, P, ctx = wc
    parity.test_commit_hash_golden(ctx)
    parity.test_trees_golden_every_node(ctx, hip_lib)
    assert sum(c["m"] <= P for c in load_golden("range.json")) >= 5
    parity.test_range_proofs_golden(ctx)                        # (skips m > ctx.max_parties itself)
    ran = 0
    for c in load_golden("dapol.json"):
        m_max = max([len(bytes.fromhex(a)) for a in c["aggregated"]] + [0])
        if any(len(bytes.fromhex(a)) > hip_lib.lib().dapol_range_proof_size(c["n_bits"], P) for a in c["aggregated"]):
            continue                                     # an aggregated sub-proof over more than P parties
        idx = np.array([l["idx"] for l in c["leaves"]], np.uint64)
        v = np.array([l["v"] for l in c["leaves"]], np.uint64)
        tr = hip_lib.Tree(ctx, c["height"], idx, v, _arr([l["r"] for l in c["leaves"]]), bytes.fromhex(c["pad_seed"]))
        pol = hip_lib.POLICY_PADDING if c["policy"] == "padding" else hip_lib.POLICY_SPLITTING
        pC, pH, out = tr.prove_entities([c["leaf"]], pol, c["agg"], c["n_bits"], bytes.fromhex(c["nonce_seed"]))
        assert out[0].tobytes().hex() == "".join(c["aggregated"]) + "".join(c["individual"]), (W, c["policy"], c["agg"], m_max)
        for s, e in enumerate(c["siblings"]):
            assert pC[0, s].tobytes().hex() == e["C"] and pH[0, s].tobytes().hex() == e["H"]
        tr.close()
        ran += 1
    assert ran == (4 if P >= 4 else 2)


# ---------------------------------------------------------------------------------------------------- C.2 commitments
def _check_commitments(ctx, pyref, W):
    """commit_hash_batch (tbl_fixed_mul_add_u64 for the value, tbl_fixed_mul_add for the blinding) over value families x blinding
    families, unreduced blindings among them, against pyref.node_new.  More than one wavefront; the random entries in front shift the
    crafted ones so that every family meets several lanes."""
    rng = np.random.default_rng(W)
    pairs = [(int(rng.integers(0, 2**63)), int.from_bytes(rng.bytes(32), "little") >> 1) for _ in range(7)]
    pairs += [(v, r) for v in _values(W) for r in _blind(W)]
    pairs += [(int(rng.integers(0, 2**63)), int.from_bytes(rng.bytes(32), "little") >> 4) for _ in range(13)]
    assert len(pairs) > 64 + 20 and sum(r >= E.L for _, r in pairs) > 20           # the crafted ones alone outnumber a wavefront
    C, H = ctx.commit_hash_batch(np.array([v for v, _ in pairs], np.uint64), _bytes32([r for _, r in pairs]))
    for i, (v, r) in enumerate(pairs):
        want = _cached(("node", v, r), lambda: pyref.node_new(v, r))
        assert C[i].tobytes() == want.C and H[i].tobytes() == want.H, (W, i, hex(v), hex(r))


def test_commitments_cross_product(wc, pyref):
    W, hi, P, ctx = wc
    _check_commitments(ctx, pyref, W)


# ---------------------------------------------------------------------------------------------------- C.3 padding nodes
def test_padding_nodes_from_crafted_tape(wc, hip_lib, pyref):
    """A tree built in tape mode whose every padding draw is a crafted canonical scalar: each padding node the tree reports is
    pyref.node_new(0, draw mod l) -- blinding, commitment and hash -- and the root is the merge over those nodes."""
    W, hi, P, ctx = wc
    height = 6
    idx = np.array([3, 4, 41], np.uint64)
    v = np.array(_values(W)[:3], np.uint64) >> np.uint64(2)            # (the root's value is their plain sum)
    rs = _blind(W)[:3]
    level, index = hip_lib.tree_padding_positions(height, idx)
    cs = _canon(W)
    draws = {(int(l), int(i)): E.draw(cs[k % len(cs)]) for k, (l, i) in enumerate(zip(level, index))}
    assert len(draws) >= len(cs)                                       # every family pads some node
    tape = b"".join(draws[(int(l), int(i))] for l, i in zip(level, index))
    tr = hip_lib.Tree(ctx, height, idx, v, _bytes32(rs), None, pad_tape=tape)
    seen = 0
    for k in range(height + 1):
        li, lv, lr, lC, lH, pad = tr.level_nodes(k)
        for j in range(len(li)):
            if not pad[j]:
                continue
            x = pyref.scalar_from_wide(draws[(k, int(li[j]))])
            want = _cached(("node", 0, x), lambda: pyref.node_new(0, x))
            assert (int(lv[j]), lr[j].tobytes(), lC[j].tobytes(), lH[j].tobytes()) == (0, E.le32(x), want.C, want.H), (W, k, int(li[j]))
            seen += 1
    assert seen == len(draws) == tr.node_count()[1]
    leaves = [(int(i), pyref.node_new(int(vv), r)) for i, vv, r in zip(idx, v, rs)]
    pt = pyref.Tree(height, leaves, draws)
    assert tr.root() == (pt.root.C, pt.root.H, pt.root.v, E.le32(pt.root.r % E.L))
    tr.close()


# ---------------------------------------------------------------------------------------------------- C.4 tree build, update, remove
@pytest.mark.parametrize("height", [12, 64])
def test_tree_build_update_remove(wc, hip_lib, ref, height):
    """Leaves whose values and blindings come from the families, among random ones, against the C oracle: root, node count, sampled
    paths; then an update that gives one leaf an `allneg` blinding and the removal of another, each against the oracle's tree over
    the resulting leaves."""
    W, hi, P, ctx = wc
    rng = np.random.default_rng(height * 100 + W)
    idx, v, r = _rand_leaves(rng, height, 48)
    vals, blinds = _values(W), _blind(W)
    for k in range(0, len(idx), 2):                                    # every other leaf is crafted
        v[k] = np.uint64(vals[(k // 2) % len(vals)] >> 6)              # (48 of them must not wrap the u64 sum the oracle checks)
        r[k] = np.frombuffer(E.le32(blinds[(k // 2) % len(blinds)]), np.uint8)
    v[1] = np.uint64(vals[0])                                          # one value at full width: the sum may wrap, as the reference's does

    def check(tr, idx, v, r, what):
        t = _ref_tree(ref, height, idx, v, r)
        assert tr.root() == _ref_root(ref, t), (W, what)
        assert sum(tr.node_count()) == ref.ref_tree_node_count(t), (W, what)
        sample = idx[::6]
        pC, pH, pv, pr = tr.paths(sample)
        for a, li in enumerate(sample):
            sC, sH, sr, sv = [ctypes.create_string_buffer(32 * height) for _ in range(3)] + [(ctypes.c_uint64 * height)()]
            assert ref.ref_tree_path(t, ctypes.c_uint64(int(li)), sC, sH, sv, sr) == 1
            assert pC[a].tobytes() == sC.raw and pH[a].tobytes() == sH.raw and pr[a].tobytes() == sr.raw and list(map(int, pv[a])) == list(sv), (W, what, a)
        ref.ref_tree_free(t)

    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    check(tr, idx, v, r, "build")
    v2, r2 = v.copy(), r.copy()
    v2[5] = np.uint64(E.families(W, "value")["allneg"] >> 6)
    r2[5] = np.frombuffer(E.le32(E.families(W, "blinding")["allneg"]), np.uint8)
    tr.update(idx[5:6], v2[5:6], r2[5:6])
    check(tr, idx, v2, r2, "update")
    keep = np.array([i for i in range(len(idx)) if i != 8])
    tr.remove(idx[8:9])
    check(tr, idx[keep], v2[keep], r2[keep], "remove")
    tr.close()


# ---------------------------------------------------------------------------------------------------- C.5 steered nonces
def _steered_case(ref, W, n, m):
    """One batch with a different crafted tape per proof, and the C oracle's proofs for it."""
    def make():
        b, slots = len(E.TAPES), m * (2 * n + 4)
        tape = np.frombuffer(b"".join(E.tape_bytes(W, name, slots) for name in E.TAPES), np.uint8)
        vals, cs = _values(W), _canon(W)
        v = np.array([vals[(i * m + j) % len(vals)] & (2**n - 1) for i in range(b) for j in range(m)], np.uint64).reshape(b, m)
        r = _bytes32([cs[(i * m + j + 1) % len(cs)] for i in range(b) for j in range(m)]).reshape(b, m, 32)
        ps = ref.ref_range_proof_size(n, m)
        out = ctypes.create_string_buffer(ps * b)
        assert ref.ref_range_prove_batch(n, m, ctypes.c_size_t(b), _p(v), _p(r), None, None, ctypes.c_uint64(0), _p(tape), 0, out) == 0
        want = np.frombuffer(out.raw, np.uint8).reshape(b, ps)
        assert want[0, 32:128].tobytes() == bytes(96)                  # the all-zero tape: S, T_1 and T_2 are the identity
        return v, r, tape, want
    return _cached(("steered", W, n, m), make)


def _check_steered(ctx, hip_lib, ref, W, hi, P):
    """Tape mode with every nonce a crafted canonical scalar, under the generator-stationary sweep (write_digits_gs) and under the
    proof-stationary latency shapes (write_digits), with and without the four-lanes-per-point kernels where the tables have the
    high-half rows those need.  Only the bytes are compared: a proof whose S is the identity does not verify."""
    for n, m in sorted({(8, 2), (64, 1), (64, P)}):
        v, r, tape, want = _steered_case(ref, W, n, m)
        for opt in (dict(generator_stationary=1, small_call_max=1), dict(generator_stationary=-1)):
            for env in (({}, {"DAPOL_NO_QUAD": "1"}) if hi > 0 else ({},)):
                ctx.set_options(hip_lib.Options(**opt))
                os.environ.update(env)
                try:
                    got = ctx.range_prove_batch(n, m, v, r, tape=tape)
                finally:
                    for k in env:
                        os.environ.pop(k, None)
                    ctx.set_options(hip_lib.Options())
                for i, name in enumerate(E.TAPES):
                    assert got[i].tobytes() == want[i].tobytes(), (W, n, m, opt, env, name)


def test_range_prove_steered_nonces(wc, hip_lib, ref):
    W, hi, P, ctx = wc
    _check_steered(ctx, hip_lib, ref, W, hi, P)


# ---------------------------------------------------------------------------------------------------- C.6 seed mode, C.7 verification
def _seed_case(ref, W, m, b):
    def make():
        rng = np.random.default_rng(1000 * W + m)
        vals = _values(W)
        v = np.array([vals[(i * m + j) % len(vals)] for i in range(b) for j in range(m)], np.uint64).reshape(b, m)
        r = rng.integers(0, 256, size=(b, m, 32), dtype=np.uint8)
        r[:, :, 31] &= 0x0F
        sid = rng.integers(0, 2**63, size=b, dtype=np.uint64)
        ps = ref.ref_range_proof_size(64, m)
        out = ctypes.create_string_buffer(ps * b)
        assert ref.ref_range_prove_batch(64, m, ctypes.c_size_t(b), _p(v), _p(r), SEED, _p(sid), ctypes.c_uint64(0), None, 0, out) == 0
        V = ctypes.create_string_buffer(32 * b * m)
        ref.ref_commit_hash(ctypes.c_size_t(b * m), _p(v), _p(r), V, ctypes.create_string_buffer(32 * b * m))
        return v, r, sid, np.frombuffer(out.raw, np.uint8).reshape(b, ps), np.frombuffer(V.raw, np.uint8).reshape(b, m, 32)
    return _cached(("seed", W, m, b), make)


def test_range_prove_seed_mode(wc, ref, gpu_ctx):
    """Values from the value families, random blindings: the oracle's bytes, and the bytes of the session's default context."""
    W, hi, P, ctx = wc
    for m, b in ((1, 16), (P, 3)):
        v, r, sid, want, _ = _seed_case(ref, W, m, b)
        got = ctx.range_prove_batch(64, m, v, r, nonce_seed=SEED, stream_id=sid)
        assert got.tobytes() == want.tobytes(), (W, m)
        dflt = _cached(("default ctx", W, m, b), lambda: gpu_ctx.range_prove_batch(64, m, v, r, nonce_seed=SEED, stream_id=sid).tobytes())
        assert got.tobytes() == dflt, (W, m)


def _fallbacks(hip_lib):
    n = ctypes.c_uint64(0)
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


def test_range_verify_both_paths(wc, hip_lib, ref):
    """range_verify_batch on seed-mode proofs of this context: all valid -> all 1; one flipped byte -> 0 for that proof alone.  16
    proofs with verify_batch_min = 2 go through the combined check (a batch with a bad proof then falls back, which the library
    counts); 3 proofs with verify_batch_min = 1000 are checked one by one (no combined check, so nothing to fall back from)."""
    W, hi, P, ctx = wc
    for m, b, vmin in ((1, 16, 2), (P, 3, 1000), (1, 3, 1000), (P, 3, 2)):
        v, r, sid, _, V = _seed_case(ref, W, m, 16 if m == 1 else 3)
        proofs = ctx.range_prove_batch(64, m, v[:b], r[:b], nonce_seed=SEED, stream_id=sid[:b])
        ctx.set_options(hip_lib.Options(verify_batch_min=vmin))
        try:
            f0 = _fallbacks(hip_lib)
            assert ctx.range_verify_batch(64, m, proofs, V[:b], verify_seed=SEED).tolist() == [1] * b, (W, m, b, vmin)
            assert _fallbacks(hip_lib) == f0
            bad = proofs.copy()
            bad[b // 2, 130] ^= 0x04                                   # a bit of t_x
            want = [1] * b
            want[b // 2] = 0
            assert ctx.range_verify_batch(64, m, bad, V[:b], verify_seed=SEED).tolist() == want, (W, m, b, vmin)
            assert (_fallbacks(hip_lib) > f0) == (b >= vmin), (W, m, b, vmin)
        finally:
            ctx.set_options(hip_lib.Options())


def _entity_case(pyref, height, name, agg):
    def make():
        rng = np.random.default_rng(height * 10 + agg)
        idx, v, r = _rand_leaves(rng, height, 5, vmax=8)
        leaves = [(int(i), pyref.node_new(int(vv), int.from_bytes(rr.tobytes(), "little"))) for i, vv, rr in zip(idx, v, r)]
        pt = pyref.Tree(height, leaves, SEED)
        return idx, v, r, pt, [pyref.dapol_prove(pt, int(idx[k]), name, agg, SEED, n=8) for k in range(2)]
    return _cached(("entity", height, name, agg), make)


def test_entity_proofs_both_policies(wc, hip_lib, pyref):
    """prove_entities / verify_entities on a height-8 tree, padding and splitting, against pyref.dapol_prove as in
    test_entity_proofs_vs_python_oracle; the aggregation factors are the largest whose sub-proofs fit the context's parties."""
    W, hi, P, ctx = wc
    height = 8
    for policy, agg in ((0, 8), (1, 5)) if P >= 8 else ((0, 2), (1, 3)):
        name = "padding" if policy == 0 else "splitting"
        idx, v, r, pt, want = _entity_case(pyref, height, name, agg)
        tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
        assert tr.root()[:2] == (pt.root.C, pt.root.H)
        pC, pH, out = tr.prove_entities(idx[:2], policy, agg, 8, SEED)
        for k in range(2):
            sibs, aggregated, individual = want[k]
            assert out[k].tobytes() == b"".join(aggregated) + b"".join(individual), (W, name, agg, k)
        lC, lH = ctx.commit_hash_batch(v[:2], r[:2])
        rC, rH, _, _ = tr.root()
        assert ctx.verify_entities(height, idx[:2], lC, lH, pC, pH, rC, rH, policy, agg, 8, out, verify_seed=SEED).tolist() == [1, 1], (W, name)
        bad = out.copy()
        bad[1, 130] ^= 0x04
        assert ctx.verify_entities(height, idx[:2], lC, lH, pC, pH, rC, rH, policy, agg, 8, bad, verify_seed=SEED).tolist() == [1, 0], (W, name)
        tr.close()


# ---------------------------------------------------------------------------------------------------- C.8 what the session fixture got
def test_session_context_width_is_covered(gpu_ctx, hip_lib, pyref, ref):
    """The session's default context chose its width from the free memory of the moment: it is one of 8..17, and if it is not one of
    the widths this module pins, the commitments and the steered nonces run at that width as well."""
    W = gpu_ctx.get_options().window_bits
    print("session gpu_ctx: window_bits = %d, high_half_rows = %d" % (W, gpu_ctx.get_options().high_half_rows))
    assert 8 <= W <= 17
    if W not in E.WIDTHS:
        for hi in (+1, -1):
            ctx = _make_ctx(hip_lib, W, hi, 8)
            try:
                _check_commitments(ctx, pyref, W)
                _check_steered(ctx, hip_lib, ref, W, hi, 8)
            finally:
                ctx.close()


def test_host_profile_width_is_16(hip_lib):
    """DAPOL_PROFILE_HOST caps the table budget at 18 GB: 16-bit windows for 32 parties (4,128 rows x 32,769 entries x 128 B =
    17.3 GB), never wider -- unless 30 % of the memory that is free right now is less than that, which lowers the width further."""
    L = hip_lib.lib()
    free_b, total_b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    hip_lib.Context(0, 1, options=hip_lib.Options(window_bits=8)).close()          # (a context has selected the device)
    assert L.hipMemGetInfo(ctypes.byref(free_b), ctypes.byref(total_b)) == 0
    need = (128 * 32 + 2 * (255 // 16 + 1)) * ((1 << 15) + 1) * 128
    assert need < 18.0e9
    faulthandler.dump_traceback_later(CTX_LIMIT_S, exit=True, file=sys.__stderr__)
    try:
        ctx = hip_lib.Context(0, 32, options=hip_lib.Options(profile=hip_lib.PROFILE_HOST))
    finally:
        faulthandler.cancel_dump_traceback_later()
    o = ctx.get_options()
    ctx.close()
    print("HOST profile, 32 parties: window_bits = %d with %.1f of %.1f GB free" % (o.window_bits, free_b.value / 1e9, total_b.value / 1e9))
    assert o.window_bits <= 16 and o.high_half_rows == -1
    if o.window_bits < 16 and 0.30 * free_b.value < need * 1.02:
        pytest.skip("free memory, not the profile, lowered the width: %.1f GB free, 30 %% of it is under the %.1f GB of 16-bit tables"
                    % (free_b.value / 1e9, need / 1e9))
    assert o.window_bits == 16
