"""The arithmetic headers as the GPU compiles them, unit by unit (tests/dev_shim.hip: one case per lane, per quad or per
wavefront), on the crafted operands of tests/limb_vectors.py.

The device does not run the code the host-path tests run: fe_mul / fe_sq are chains of v_mad_i64_i32 / v_mad_u64_u32 in inline
assembly, sc_redc29 goes through sc_mad's v_mad_u64_u32, ge_quad.h (a point per four lanes, DPP quad permutes) and the
wavefront-held STROBE of hash.h have no host form at all.  Every case must equal the big-integer / pyref value, keep the
output-limb contract of fe.h (test_limb_bounds_cpu.py) and equal the HOST path limb for limb; every wrapper must return
hipSuccess.  A mismatch is a failing assertion, never a fault: the kernels take no input outside the headers' preconditions."""
import ctypes

import numpy as np
import pytest

import arith_checks as C
import arith_shim as A
import limb_vectors as V


def test_device_program_cross_compiles():
    """no device needed: hipcc builds tests/dev_shim.hip for gfx950 with the library's flags, and the wrappers are there"""
    lib = ctypes.CDLL(A.build_dev_shim())
    for name in ("fe_cases", "ge_cases", "ge_decompress_cases", "ge_uniform_cases", "sc_cases", "sc_wide_cases", "sc_recode_cases",
                 "quad_cases", "strobe_cases"):
        assert hasattr(lib, "d_" + name)


@pytest.fixture(scope="module")
def dev():
    return A.Cases(ctypes.CDLL(A.build_dev_shim()), "d_")


@pytest.fixture(scope="module")
def host(host_shim):
    return A.Cases(host_shim, "t_")


@pytest.mark.gpu
def test_fe_mul_sq_chains_at_the_limb_bounds(dev, host):
    """the madNz / madNclh chains: value, contract, the Python column model and the host path's C sums, limb for limb"""
    assert C.fe_mul(dev) == C.fe_mul(host)
    assert C.fe_sq(dev) == C.fe_sq(host)


@pytest.mark.gpu
def test_fe_carry_addc_towords(dev, host):
    assert C.fe_carry(dev) == C.fe_carry(host)
    assert C.fe_addc(dev) == C.fe_addc(host)
    assert C.fe_towords(dev) == C.fe_towords(host)
    prods = C.fe_mul(host)[::3]
    assert C.fe_abs(dev, prods) == C.fe_abs(host, prods)


@pytest.mark.gpu
def test_fe_invert_pow_sqrt_ratio(dev, host, pyref):
    assert C.fe_powers(dev) == C.fe_powers(host)
    assert C.fe_sqrt_ratio(dev, pyref) == C.fe_sqrt_ratio(host, pyref)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [A.GE_MADD, A.GE_ADD, A.GE_DBL, A.GE_ADD_CACHED, A.GE_NEG, A.GE_CHAIN])
def test_group_ops_one_point_per_lane(dev, host, pyref, op):
    assert C.ge_op(dev, pyref, op) == C.ge_op(host, pyref, op)


@pytest.mark.gpu
def test_codec_one_point_per_lane(dev, host, pyref):
    assert C.ge_codec(dev, pyref) == C.ge_codec(host, pyref)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [A.GE_MADD, A.GE_ADD, A.GE_DBL, A.GE_ADD_CACHED, A.GE_CHAIN])
def test_group_ops_one_point_per_four_lanes(dev, pyref, op):
    """ge_quad.h in whole wavefronts (16 points each; the cases are repeated until they fill more than one wavefront, with a
    ragged tail): against pyref, and coordinate for coordinate in VALUE against the per-lane ge_* result on the same inputs --
    the two reach the same X, Y, Z, T by the same formulas, so equal values, not merely the same point."""
    triples, negs = C.ge_cases_of(pyref, op)
    triples = (triples * 3)[:len(triples) * 2 + 5]
    cases, quad = C._run_ge(dev, pyref, op, triples, negs, quad=True)
    _, (lane, _) = C._run_ge(dev, pyref, op, triples, negs)
    assert len(cases) > 16 and len(cases) % 16
    for (name, p, q, ng), ql, ll in zip(cases, quad.tolist(), lane.tolist()):
        want = C.ge_expected(pyref, op, p, q, ng)
        got = V.point_of_limbs(pyref, ql)
        assert got == want and got.compress() == want.compress(), (op, name, ng)
        assert (got.X * got.Y - got.Z * got.T) % V.P == 0, (op, name, ng)             # T is consistent (the encoding reads it)
        for k in range(4):
            assert V.value(ql[9 * k:9 * k + 9]) % V.P == V.value(ll[9 * k:9 * k + 9]) % V.P, (op, name, ng, "XYZT"[k])
            assert V.contract_ok(ql[9 * k:9 * k + 9], V.MUL_LIMB1), (op, name, ng, "XYZT"[k])


@pytest.mark.gpu
def test_scalar_ops(dev, host):
    """sc_montmul (sc_mad's v_mad_u64_u32 in the reduction), add, sub, from_wide, both inversions, from_u64, sc_recode_w at
    edge_scalars.WIDTHS: against Python integers and edge_scalars.recode, and word for word against the host path"""
    assert C.scalars(dev) == C.scalars(host)


@pytest.fixture(scope="module")
def strobe_run(dev):
    return C.strobe_run(dev)                           # one launch: a block (WStrobe wavefront + one-lane Strobe) per case


@pytest.mark.gpu
def test_wavefront_strobe_reaches_every_block_position(strobe_run):
    """k = 0..165 filler bytes put the first word of the message at every position of the 166-byte block -- the in-block fast
    path of strobe_absorb_word on every lane boundary, the exact end (162) and the byte fallback (163..165) -- and the
    wavefront's state gives the challenges the one-lane Strobe gives on another wavefront of the same block"""
    _, _, _, out, pos = strobe_run
    C.strobe_positions(strobe_run, 0)
    assert (pos[:, 0] == pos[:, 1]).all()
    assert (out[:, 0] == out[:, 1]).all(), np.nonzero((out[:, 0] != out[:, 1]).any(axis=1))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", C.STROBE_NWORDS)
def test_wavefront_strobe_against_merlin(strobe_run, pyref, n):
    C.strobe_against_merlin(strobe_run, pyref, n, 0)
