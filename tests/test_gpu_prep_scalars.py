"""The digit producers of the swept prover under DAPOL_PREP=v2 -- the unrolled recode of the compiled window geometries
(write_digits_gs -> sc_recode_fixed) and the materialisation's scalars written once per (side, k) with y^-i left to the tail
(k_rp_mat_prep_gs_shared, k_rp_mat_gs, tail_row_vectors; dapol_amd/csrc/kernels_range_gs.h, kernels_range.h) -- against the
producers as they were (DAPOL_PREP=v1) and the C oracle, byte for byte, at the smallest shapes at which each part can go wrong.
Every case first asks the plan (a host build of prove_plan.inc, tests/cpp/prep_plan_host.cpp, fed with the context's geometry)
that the call really is swept, materialises swept, runs in table mode and takes the new producers under v2 and the old under v1:
a forced knob that the plan ignored would compare a kernel with itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_scalars as E
from conftest import ROOT
from test_gpu_full_range import _leaves, _oracle_entity_blob
from test_gpu_tail_order import SEED, _inputs, _oracle, _plan, _with_env

pytestmark = pytest.mark.gpu
V1, V2 = {"DAPOL_PREP": "v1"}, {"DAPOL_PREP": "v2"}
# the generator-stationary sweep for any batch size: forced on, with the latency shapes of small calls out of the way (a call of one
# proof is a small call at any DAPOL_SMALL_MAX >= 1 unless its split is refused)
SWEEP = {"DAPOL_GS": "1", "DAPOL_SMALL_MAX": "1"}


def _sweep(b):
    return dict(SWEEP, DAPOL_NO_SPLIT="1") if b == 1 else SWEEP


def _p(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def plan_exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "prep_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "prep_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _check_plans(exe, ctx, n_bits, m, b, env, tail_n, table_mode=True, stab_tail=None):
    """v2: swept, the new recode, and -- with a tail in table mode -- the shared scalars; v1: the same call with neither."""
    new, old = _plan(exe, ctx, n_bits, m, b, dict(env, **V2)), _plan(exe, ctx, n_bits, m, b, dict(env, **V1))
    for p in (new, old):
        assert p["gs"] == 1 and p["small_call"] == 0 and p["tail_n"] == tail_n, p
        assert p["gs_mat"] == (1 if tail_n else 0) and p["stab_main"] == (1 if table_mode else 0), p
        if stab_tail is not None:
            assert p["stab_tail"] == stab_tail, p
    assert new["prep_recode"] == 1 and new["prep_share"] == (1 if tail_n and table_mode else 0), new
    assert old["prep_recode"] == 0 and old["prep_share"] == 0, old
    for k in ("chunk", "dig_elems", "per_proof", "lane_bytes", "acc_bytes", "stab_bytes"):
        assert new[k] == old[k], k
    return new


# (n_bits, parties, tail length, extra knobs, table mode)
SHAPES = [(64, 32, 64, {}, True),                              # N = 2,048, five main rounds: the headline's own table depth
          (32, 32, 64, {}, True), (64, 16, 64, {}, True),      # N = 1,024, four main rounds
          (64, 8, 32, {"DAPOL_TAIL_N": "32"}, True),           # N = 512, T = 32: the short-list sweep (two lookups a term)
          (64, 1, 0, {}, True),                                # no tail: the recode alone, tables all the way
          (64, 32, 64, {"DAPOL_NO_STAB": "1"}, False)]         # vector mode: the scalars stay per generator


@pytest.mark.parametrize("n_bits,m,tail_n,extra,table_mode", SHAPES)
def test_every_shape_gives_the_same_bytes_with_either_producers(gpu_ctx, ref, plan_exe, n_bits, m, tail_n, extra, table_mode):
    b = 5
    env = dict(_sweep(b), **extra)
    _check_plans(plan_exe, gpu_ctx, n_bits, m, b, env, tail_n, table_mode, stab_tail=(1 if tail_n and table_mode else 0))
    v, r, sid = _inputs(n_bits, m, b, 77 * n_bits + m)
    prove = lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid)
    old = _with_env(dict(env, **V1), prove)
    new = _with_env(dict(env, **V2), prove)
    assert new.tobytes() == old.tobytes()
    for i in (0, b - 1):
        assert new[i].tobytes() == _oracle(ref, n_bits, m, v, r, sid, i), i


@pytest.fixture(scope="module")
def batch67(gpu_ctx, ref):
    """67 proofs of 32 bits x 32 parties (N = 1,024, T = 64) from the old producers, computed once; the oracle's first and last."""
    n_bits, m, b = 32, 32, 67
    v, r, sid = _inputs(n_bits, m, b, 167)
    old = _with_env(dict(SWEEP, **V1), lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid))
    assert old[0].tobytes() == _oracle(ref, n_bits, m, v, r, sid, 0) and old[b - 1].tobytes() == _oracle(ref, n_bits, m, v, r, sid, b - 1)
    old.setflags(write=False)
    return n_bits, m, v, r, sid, old


@pytest.mark.parametrize("b", [1, 5, 17, 67])
def test_batch_sizes_around_the_producer_quads(gpu_ctx, plan_exe, batch67, b):
    """Producer lanes come in quads of sweep positions, 16 proofs a wavefront: one proof, a partly filled wavefront, one wavefront
    and a proof, four and three.  A proof's bytes do not depend on its batch, so every size is a prefix of the one reference."""
    n_bits, m, v, r, sid, old = batch67
    env = _sweep(b)
    _check_plans(plan_exe, gpu_ctx, n_bits, m, b, env, 64)
    new = _with_env(dict(env, **V2), lambda: gpu_ctx.range_prove_batch(n_bits, m, v[:b], r[:b], nonce_seed=SEED, stream_id=sid[:b]))
    assert new.tobytes() == old[:b].tobytes()


def test_two_chunks_with_a_short_last_one(gpu_ctx, plan_exe, batch67):
    """DAPOL_CHUNK=64 cuts 67 proofs into a full chunk and one of three through the same digit buffer: the shared scalars sit at
    positions that depend on the chunk's own proof count."""
    n_bits, m, v, r, sid, old = batch67
    env = dict(SWEEP, DAPOL_CHUNK="64")
    assert _check_plans(plan_exe, gpu_ctx, n_bits, m, 67, env, 64)["chunk"] == 64
    new = _with_env(dict(env, **V2), lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid))
    assert new.tobytes() == old.tobytes()


def _edge_scalars(W):
    """Canonical scalars on every edge of the signed recoding at width W: 0, 1, l - 1, the families of tests/edge_scalars.py, and for
    every window boundary 2^(W i) - 1 / + 0 / + 1 (all ones below: a carry arrives), the same with window i at half already, and the
    carry chain through all windows (`allneg`) with window i pushed one up (the chain goes on) and one down (it ends there)."""
    fam = E.families(W, "canonical")
    xs = [0, 1, E.L - 1] + [fam[k] for k in sorted(fam)]
    k, half = E.whole_windows("canonical", W), 1 << (W - 1)
    for i in range(1, E.nwin_of("canonical", W)):
        bnd = 1 << (W * i)
        xs += [bnd - 1, bnd, bnd + 1, bnd - 1 + (half << (W * i))]
        if i < k:
            xs += [fam["allneg"] + bnd, fam["allneg"] - bnd, fam["allneg"] - (bnd >> 1)]
    xs = sorted({x for x in xs if 0 <= x < E.L})
    for x in xs:                                                       # (what the list is for: it reaches both ends of the digit range)
        assert sum(d << (W * i) for i, d in enumerate(E.recode(x, W, E.nwin_of("canonical", W)))) == x
    digs = [d for x in xs for d in E.recode(x, W, E.nwin_of("canonical", W))]
    assert min(digs) == -half and max(digs) >= half - 1
    return xs


@pytest.mark.parametrize("W,parties,fixed", [(17, 4, True), (16, 4, True), (11, 2, False)])
def test_steered_nonces_on_every_edge_of_the_recode(hip_lib, ref, plan_exe, W, parties, fixed):
    """Tape mode with every nonce a crafted canonical scalar (as test_range_prove_steered_nonces): the S commitment's digits are the
    recoding of the tape's own scalars, so they hit every branch of the unrolled recode -- at 17 and 16 bits, and at 11 bits, which
    keeps the loop.  Three proofs, the list of scalars shifted by one slot from proof to proof; against the oracle and the old
    producers.  Only bytes are compared."""
    n, m, b = 64, parties, 3
    assert ((W, 253 // W + 1) in ((17, 15), (16, 16))) == fixed
    ctx = hip_lib.Context(0, parties, options=hip_lib.Options(window_bits=W, high_half_rows=-1))
    try:
        assert ctx.get_options().window_bits == W
        N = n * m
        _check_plans(plan_exe, ctx, n, m, b, SWEEP, 64 if N >= 256 else 0)
        xs, slots = _edge_scalars(W), m * (2 * n + 4)
        assert len(xs) < 2 * N                                         # every scalar is some s_L / s_R of every proof
        tape = np.frombuffer(b"".join(E.draw(xs[(s + i) % len(xs)]) for i in range(b) for s in range(slots)), np.uint8)
        rng = np.random.default_rng(W)
        v = rng.integers(0, 2**63, size=(b, m), dtype=np.uint64)
        r = rng.integers(0, 256, size=(b, m, 32), dtype=np.uint8)
        r[:, :, 31] &= 0x0F
        ps = ref.ref_range_proof_size(n, m)
        out = ctypes.create_string_buffer(ps * b)
        assert ref.ref_range_prove_batch(n, m, ctypes.c_size_t(b), _p(v), _p(r), None, None, ctypes.c_uint64(0), _p(tape), 0, out) == 0
        prove = lambda: ctx.range_prove_batch(n, m, v, r, tape=tape)
        new = _with_env(dict(SWEEP, **V2), prove)
        assert new.tobytes() == out.raw
        assert _with_env(dict(SWEEP, **V1), prove).tobytes() == out.raw
    finally:
        ctx.close()


def test_splitting_policy_at_height_32(gpu_ctx, hip_lib, ref, pyref, plan_exe):
    """prove_entities under the splitting policy at height 32 with aggregation factor 24: every entity is one proof of 16 parties,
    one of 8 and eight individual ones (N = 1,024, 512 and 64: the swept materialisation, the short-list sweep and a swept call
    without a tail), all through the policy's lane runner; the first and the last entity against the oracle's prover."""
    height, agg = 32, 24
    rng = np.random.default_rng(3224)
    idx, v, r = _leaves(rng, height, 5, vmax=2**40)
    _check_plans(plan_exe, gpu_ctx, 64, 16, len(idx), SWEEP, 64)
    _check_plans(plan_exe, gpu_ctx, 64, 8, len(idx), SWEEP, 64)
    tr = hip_lib.Tree(gpu_ctx, height, idx, v, r, SEED)
    try:
        prove = lambda: tr.prove_entities(idx, hip_lib.POLICY_SPLITTING, agg, 64, SEED)
        pC, pH, new = _with_env(dict(SWEEP, **V2), prove)
        _, _, old = _with_env(dict(SWEEP, **V1), prove)
        assert new.tobytes() == old.tobytes()
        _, _, sv, sr = tr.paths(idx)
        for k in (0, len(idx) - 1):
            want = _oracle_entity_blob(ref, pyref, np.ascontiguousarray(sv[k]), np.ascontiguousarray(sr[k]), 1, agg, 64, idx[k])
            assert new[k].tobytes() == want, k
    finally:
        tr.close()
