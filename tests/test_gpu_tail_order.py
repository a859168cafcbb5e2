"""The tail rounds of the hybrid inner-product argument with a lane per (proof, list, window) -- k_rp_tail_gs + k_rp_tail_combine
(dapol_amd/csrc/kernels_range_gs.h), DAPOL_TAIL_ORDER=gs -- against the proof-stationary kernel (DAPOL_TAIL_ORDER=ps) and the C
oracle, byte for byte, at the smallest shapes at which the new order can go wrong: every tail length / list length it serves, batch
sizes around the packing of 51-lane lists into 256-thread blocks (5 lists = 2.5 proofs a block), a multi-chunk call with a short
last chunk, and enough random proofs for every digit value of the 5-bit windows.  Each case first asks the plan (a host build of
prove_plan.inc, tests/cpp/tail_order_plan_host.cpp, fed with the context's geometry) whether the call really has a tail and really
takes the new order: a forced knob that the plan ignored would compare a kernel with itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
GS, PS = {"DAPOL_TAIL_ORDER": "gs"}, {"DAPOL_TAIL_ORDER": "ps"}


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def plan_exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tail_order_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tail_order_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _plan(exe, ctx, n_bits, m, b, env):
    """The plan of ctx.range_prove_batch(n_bits, m, <b proofs>) under the knobs `env` (chunking aside, which needs the device's
    free memory: the calls here are far below one chunk of any budget)."""
    o = ctx.get_options()
    nwin = 253 // o.window_bits + 1
    shape = {"n": n_bits, "m": m, "B": b, "opt_tail_length": o.tail_length, "opt_small_call_max": o.small_call_max,
             "opt_generator_stationary": o.generator_stationary, "opt_streams": o.streams, "opt_chunk_proofs": o.chunk_proofs,
             "opt_gs_tile_rows": o.gs_tile_rows, "opt_gs_slices": o.gs_slices, "wbits": o.window_bits, "nwin": nwin,
             "hi_split": (nwin + 1) // 2 if o.high_half_rows > 0 else 0, "n_cu": 256, "resident_waves": 4096, "budget_bytes": 16 << 30, "timed": 0}
    line = " ".join(["%s=%s" % kv for kv in env.items()] + ["%s=%d" % kv for kv in shape.items()])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DAPOL_")}
    r = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, timeout=60, env=clean)
    assert r.returncode == 0, r.stderr
    return {t.split("=")[0]: int(t.split("=")[1]) for t in r.stdout.split()}


def _inputs(n_bits, m, b, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**n_bits if n_bits < 64 else 2**63, size=(b, m), dtype=np.uint64)
    r = rng.integers(0, 256, size=(b, m, 32), dtype=np.uint8)
    r[:, :, 31] &= 0x0F
    sid = rng.integers(0, 2**62, size=b, dtype=np.uint64)
    return v, r, sid


def _oracle(ref, n_bits, m, v, r, sid, i):
    """Proof i of the batch from the C oracle (its own stream, slot 0)."""
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    out = ctypes.create_string_buffer(ref.ref_range_proof_size(n_bits, m))
    vi, ri, si = np.ascontiguousarray(v[i]), np.ascontiguousarray(r[i]), np.ascontiguousarray(sid[i:i + 1])
    assert ref.ref_range_prove_batch(n_bits, m, ctypes.c_size_t(1), p(vi), p(ri), SEED, p(si), ctypes.c_uint64(0), None, 0, out) == 0
    return out.raw


def _check_plans(exe, ctx, n_bits, m, b, extra, tail_n):
    """Forced gs: a tail of the expected length in the new order; forced ps: the same tail in the old one."""
    g, s = _plan(exe, ctx, n_bits, m, b, dict(extra, **GS)), _plan(exe, ctx, n_bits, m, b, dict(extra, **PS))
    assert g["tail_n"] == s["tail_n"] == tail_n, (g, s)
    assert g["tail_gs"] == 1 and s["tail_gs"] == 0, (g, s)
    assert g["acc_bytes"] + g["tail_rec_bytes"] >= g["tail_rec_need"], g          # the records of a round fit the chunk's accumulators
    assert s["tail_rec_bytes"] == 0 and g["acc_bytes"] == s["acc_bytes"], (g, s)
    return g


# DAPOL_SMALL_TAIL: calls of up to 32 proofs skip the tail argument otherwise (prove_plan.inc) -- nothing to test without one
SMALL = {"DAPOL_SMALL_TAIL": "1"}


@pytest.mark.parametrize("n_bits,m,tail_n,extra", [(64, 32, 64, {}), (64, 16, 64, {}), (32, 32, 64, {}), (64, 8, 32, {"DAPOL_TAIL_N": "32"})])
def test_every_tail_shape_gives_the_same_bytes_in_both_orders(gpu_ctx, ref, plan_exe, n_bits, m, tail_n, extra):
    """T = 64 over N = 2,048 and over N = 1,024 (two ways), T = 32 over N = 512: six proofs (a full block of five lists, a second
    one and a partial third), all against the proof-stationary order, the first and the last against the oracle."""
    b = 6
    env = dict(SMALL, **extra)
    _check_plans(plan_exe, gpu_ctx, n_bits, m, b, env, tail_n)
    v, r, sid = _inputs(n_bits, m, b, 1000 * n_bits + m)
    prove = lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid)
    old = _with_env(dict(env, **PS), prove)
    new = _with_env(dict(env, **GS), prove)
    assert new.tobytes() == old.tobytes()
    for i in (0, b - 1):
        assert new[i].tobytes() == _oracle(ref, n_bits, m, v, r, sid, i), i


@pytest.fixture(scope="module")
def batch67(gpu_ctx, ref):
    """67 proofs of 32 bits x 32 parties (N = 1,024, T = 64) in the proof-stationary order, computed once; the oracle's first and last."""
    n_bits, m, b = 32, 32, 67
    v, r, sid = _inputs(n_bits, m, b, 67)
    old = _with_env(PS, lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid))
    assert old[0].tobytes() == _oracle(ref, n_bits, m, v, r, sid, 0) and old[b - 1].tobytes() == _oracle(ref, n_bits, m, v, r, sid, b - 1)
    old.setflags(write=False)
    return n_bits, m, v, r, sid, old


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6, 67])
def test_list_packing_at_every_batch_size(gpu_ctx, plan_exe, batch67, b):
    """A block holds five whole lists = 2.5 proofs: one proof (two lists, a partial block), two (a partial block of four), 2.5
    proofs exactly (b = 5: two full blocks), and one list more or less around full blocks (b = 3: one full block + one list;
    b = 4, 6); 67 proofs = 26 full blocks + four lists, more than one wavefront round of nothing.  A proof's bytes do not depend on
    the batch it is proved in, so every size is a prefix of the one proof-stationary reference."""
    n_bits, m, v, r, sid, old = batch67
    env = SMALL if b <= 32 else {}
    _check_plans(plan_exe, gpu_ctx, n_bits, m, b, env, 64)
    new = _with_env(dict(env, **GS), lambda: gpu_ctx.range_prove_batch(n_bits, m, v[:b], r[:b], nonce_seed=SEED, stream_id=sid[:b]))
    assert new.tobytes() == old[:b].tobytes()


@pytest.mark.parametrize("chunk_proofs,b,chunk", [(8, 21, 21), (64, 67, 64)])
def test_chunked_calls_with_a_short_last_chunk(hip_lib, plan_exe, batch67, chunk_proofs, b, chunk):
    """The context option chunk_proofs on a fresh context of 12-bit tables (22 windows a scalar, other accumulator sizes).  The plan
    never cuts chunks below 64 proofs, so chunk_proofs = 8 leaves 21 proofs in ONE chunk (asserted: the case is kept as a call that
    asks for chunks and gets none); chunk_proofs = 64 splits 67 proofs into a full chunk and a last one of three through one record
    area -- the kernels' bounds are the chunk's own proof count, and the chunk before leaves 64 proofs' records behind."""
    n_bits, m, v, r, sid, old = batch67
    ctx = hip_lib.Context(0, 32, options=hip_lib.Options(window_bits=12, chunk_proofs=chunk_proofs))
    env = SMALL if b <= 32 else {}
    g = _check_plans(plan_exe, ctx, n_bits, m, b, env, 64)
    assert g["chunk"] == chunk
    new = _with_env(dict(env, **GS), lambda: ctx.range_prove_batch(n_bits, m, v[:b], r[:b], nonce_seed=SEED, stream_id=sid[:b]))
    assert new.tobytes() == old[:b].tobytes()


@pytest.mark.parametrize("n_bits,m,tail_n,extra", [(64, 32, 64, {}), (64, 8, 32, {"DAPOL_TAIL_N": "32"})])
@pytest.mark.parametrize("b", [1, 3, 5])
def test_four_table_rows_a_lane_give_the_same_bytes(gpu_ctx, ref, plan_exe, n_bits, m, tail_n, extra, b):
    """k_rp_tail_table4 (DAPOL_TAIL_ROWS_PER_LANE=4: one field inversion per four rows of a proof's tail table) against one row a
    lane and against the oracle: 128 rows a proof (T = 64: 32 lanes a proof, two proofs a wavefront) and 64 rows (T = 32: 16 lanes,
    four proofs a wavefront), with one, three and five proofs -- a partly filled wavefront, and a proof or a proof's half past
    the last.  Every tail length is a power of two >= 32, so no plan has a row count that four does not divide (the plan would
    answer 1: asserted on the CPU, tests/test_tail_order_plan_cpu.py)."""
    env = dict(SMALL, **extra)
    four, one = dict(env, DAPOL_TAIL_ROWS_PER_LANE="4"), dict(env, DAPOL_TAIL_ROWS_PER_LANE="1")
    p4, p1 = _plan(plan_exe, gpu_ctx, n_bits, m, b, four), _plan(plan_exe, gpu_ctx, n_bits, m, b, one)
    assert p4["tail_n"] == p1["tail_n"] == tail_n and p4["tail_rpl"] == 4 and p1["tail_rpl"] == 1, (p4, p1)
    v, r, sid = _inputs(n_bits, m, b, 4000 + 10 * m + b)
    prove = lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid)
    new = _with_env(four, prove)
    assert new.tobytes() == _with_env(one, prove).tobytes()
    assert new.tobytes() == _with_env(dict(four, **GS), prove).tobytes()                 # ... and feeding the other order of the rounds
    for i in sorted({0, b - 1}):
        assert new[i].tobytes() == _oracle(ref, n_bits, m, v, r, sid, i), i


def test_every_digit_value_of_the_tail_windows(gpu_ctx, plan_exe):
    """The tail's scalars are products of folded vector entries and challenge coefficients: no input puts a chosen digit there, so
    the crafted scalars of tests/edge_scalars.py do not reach them.  64 random proofs of 64 bits x 32 parties instead: 64 proofs x 6
    rounds x 128 terms x 51 windows = 2.5 million digits, each value of -16 ... +16 some 76,000 times (the ends half as often)."""
    n_bits, m, b = 64, 32, 64
    _check_plans(plan_exe, gpu_ctx, n_bits, m, b, {}, 64)
    v, r, sid = _inputs(n_bits, m, b, 5)
    prove = lambda: gpu_ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=sid)
    assert _with_env(GS, prove).tobytes() == _with_env(PS, prove).tobytes()
