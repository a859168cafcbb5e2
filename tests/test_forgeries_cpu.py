"""tests/golden/forgeries.json on the CPU: range proofs that are consistent in the transcript and wrong in the algebra only
(tests/golden/gen_forgeries.py; oracle/pyref.py range_prove(forge=)).  "Rejected" here means rejected BY AN EQUATION: every row
replays the prover's challenges exactly and leaves a non-identity residual in the half of the check its `violates` field names
(t: the polynomial equation the verifier weighs by c; P: the inner-product equation) and the identity in the other.  Both oracles
must reject every row and accept the honest proof of each shape; the GPU paths see the same rows in tests/test_gpu_forgeries.py."""
import ctypes
import os
import sys

import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import gen_forgeries as GF  # noqa: E402

IDENT = bytes(32)
ONE = bytes([1]) + bytes(31)


@pytest.fixture(scope="module")
def rows():
    return load_golden("forgeries.json")["rows"]


def _by_shape(rows, m):
    return [r for r in rows if r["m"] == m]


def test_fixture_covers_every_kind_at_every_shape(rows, pyref):
    assert os.path.getsize(os.path.join(GOLDEN, "forgeries.json")) < 200 * 1000
    for n, m in GF.SHAPES:
        mine = _by_shape(rows, m)
        assert {r["kind"] for r in mine} == set(pyref.FORGE_KINDS) | {"honest"}, (n, m)
        assert [r["kind"] for r in mine].count("honest") == 1
        N, lb = n * m, ((n * m).bit_length() - 1) // 2
        assert {r["position"]["q"] for r in mine if r["kind"] == "bit"} == {0, (1 << lb) - 1, 1 << lb, N - 1}
        assert {r["position"]["q"] for r in mine if r["kind"] == "a_R"} >= {(1 << lb) - 1, 1 << lb}          # (all four at (8,1))
        for gen in ("G", "H"):                      # every generator position is moved once on each side, by A, S, L_k or R_k
            assert {r["position"]["q"] for r in mine if r["position"].get("P") == gen} == {0, (1 << lb) - 1, 1 << lb, N - 1}
        for kind in ("L_k", "R_k"):
            assert {r["position"]["k"] for r in mine if r["kind"] == kind} == {0, N.bit_length() - 2}
        assert {r["position"]["party"] for r in mine if r["kind"] == "value"} == {0, m - 1} | ({3} if m == 8 else set())
        assert {r["position"]["party"] for r in mine if r["kind"] == "blinding"} == {0, m - 1}
        assert {r["d"] for r in mine if r["kind"] == "value"} == {"1", "L-1", "2^n"}
        assert {r["d"] for r in mine if r["kind"] not in ("value", "honest")} == {"1", "L-1"}


@pytest.mark.parametrize("m", [1, 4, 8])
def test_python_oracle_rejects_by_the_named_equation(rows, pyref, m):
    """range_verify under its default c and under c = 1, and the violated-equation field re-derived from the residuals of
    range_verify(info=): acc(0) for P, acc(1) - acc(0) for t; the stored closed forms are those residuals."""
    for r in _by_shape(rows, m):
        proof, Vs = bytes.fromhex(r["proof"]), [bytes.fromhex(V) for V in r["commitments"]]
        honest = r["kind"] == "honest"
        info = {}
        ok, res_P, res_t = pyref.range_verify(proof, Vs, r["n"], info=info)
        assert ok == honest, r["kind"]
        assert pyref.range_verify(proof, Vs, r["n"], c=1) == honest
        if honest:
            assert res_P == IDENT and res_t == IDENT
            continue
        assert GF.violated(res_P, res_t) == r["violates"], (r["kind"], r["position"])
        # acc(c) = acc_P + c acc_t with the default c: not the identity, whichever half holds (the scalar multiple of a non-identity
        # point of prime order by c != 0 is not the identity, and for `both` the generator's closed forms show -d B c + w d B != 0)
        for half, got in (("P", res_P), ("t", res_t)):
            if half in r["predicted"]:
                assert bytes.fromhex(r["predicted"][half]) == got != IDENT


def test_c_oracle_rejects_every_row(rows, ref):
    for r in rows:
        proof, V = bytes.fromhex(r["proof"]), b"".join(bytes.fromhex(V) for V in r["commitments"])
        for c32 in (ONE, bytes([7]) + bytes(31), bytes(range(1, 32)) + bytes([0])):
            got = ref.ref_range_verify(r["n"], r["m"], proof, ctypes.c_size_t(len(proof)), V, c32, 0)
            assert got == (1 if r["kind"] == "honest" else 0), (r["kind"], r["position"], c32[:2])


def test_the_generator_reproduces_the_8x1_rows(rows):
    again = GF.rows_for_shape(8, 1)
    assert again == _by_shape(rows, 1)
