"""The limb arithmetic of dapol_amd/csrc/fe.h / ge.h / sc.h on RAW limbs at the bounds its contract states, on the host path
(the headers compiled by g++: the C sums, not the device's v_mad chains -- tests/test_gpu_device_arith.py runs the same vectors
there).  Values against big integers, output limbs against the contract fe.h states:

    limbs 0, 2..7 in [0, 2^29), limb 8 in [0, 2^23), limb 1 in [lo, 2^29 - 1 + hi] with
    (lo, hi) = (-32849, 32849) after fe_mul (f loose, g tight), (-9733, 10950) after fe_sq (f tight), (-1, 1) after fe_carry.

The (lo, hi) are DERIVED (limb_vectors.limb1_excess_*: interval arithmetic over the column sums from the input bounds alone) and
the first test pins the derivation to the numbers; the families are shown here to reach the edges they are named after."""
import pytest

import arith_checks as C
import arith_shim as A
import limb_vectors as V


@pytest.fixture(scope="module")
def host(host_shim):
    return A.Cases(host_shim, "t_")


def test_contract_numbers_follow_from_the_input_bounds():
    assert V.limb1_excess_mul() == V.MUL_LIMB1 and V.limb1_excess_sq() == V.SQ_LIMB1
    # every reduced limb is TIGHT with room to spare, and so is the difference of two reduced values (Y - X in ge.h)
    lo, hi = V.MUL_LIMB1
    assert V.M29 + hi < V.TIGHT and (V.M29 + hi) - lo == 2**29 - 1 + 65698 <= V.TIGHT
    # fe_mul's columns at the stated bounds fit int64: nine products of 3 T^2, the carry and the wrapped high half
    raw, chained = V.columns_mul([V.LOOSE] * 9, [V.TIGHT] * 9)
    assert max(chained) < 2**63 * 0.85 and max(raw) == 27 * V.TIGHT**2


def test_families_reach_their_edges():
    # a column at its bound, either sign, both as the plain sum of its products and as the chained int64 the code holds
    for k, sigma, f, g in V.column_extreme_pairs():
        raw, chained = V.columns_mul(f, g)
        bound = len([i for i in range(9) if 0 <= k - i < 9]) * V.LOOSE * V.TIGHT
        assert raw[k] == sigma * bound
        if k <= 8:
            assert sigma * chained[k] >= 0.9 * bound, (k, sigma)
        if k == 8:                                               # ... and with it what limb 1 receives from the top, t >> 29
            t29 = ((chained[8] >> 23) * 19 + (chained[0] & V.M29)) >> 29
            assert t29 * sigma >= 0.9 * V.MUL_LIMB1[1], (sigma, t29)
    for k, sigma, f in V.square_column_inputs():
        raw, chained = V.columns_sq(f)
        n = len([i for i in range(9) if 0 <= k - i < 9])
        bound = (n if sigma > 0 else n - (k % 2 == 0)) * V.TIGHT**2
        assert raw[k] == sigma * bound and (k > 8 or sigma * chained[k] >= 0.9 * bound), (k, sigma)
    # negative high columns whose low half is at either end
    zones = set()
    for k, zone, f, g in V.high_split_pairs():
        col = V.raw_columns_mul(f, g)[k]
        lo = col & 0xFFFFFFFF
        assert col < -2**58 and {"zero": lo == 0, "low": 0 < lo < 16, "high": 2**32 - 16 < lo < 2**32 - 1, "ones": lo == 2**32 - 1}[zone]
        zones.add((k, zone))
    assert len(zones) == 8 * 4
    pairs = V.field_pairs()
    assert any(f[8] >= 2**23 for fam, f, _ in pairs if fam == "limb8") and any(f[8] <= -2**23 for fam, f, _ in pairs if fam == "limb8")
    assert {fam for fam, _, _ in pairs} == {"allmax", "column", "hisplit", "neglimb1", "poslimb1", "limb8", "special", "random"}


def test_other_families_reach_their_edges(pyref):
    sp = V.special_limbs()
    assert [V.value(sp[k]) for k in ("zero", "one", "p-1", "p")] == [0, 1, V.P - 1, V.P]
    assert max(max(map(abs, f)) for _, f in V.square_inputs()) == V.TIGHT
    by = {}
    for fam, f in V.carry_inputs():
        by[fam] = max(by.get(fam, 0), max(map(abs, f)))
    assert (by["stated"], by["loose"], by["full"]) == (2**31 // 20, V.LOOSE, 2**31 - 5)
    enc = V.encoding_inputs()
    assert {0, 1, V.P - 1, 19, V.P - 19} <= {v for v, _ in enc}                       # 0 = 0, p, 2p; p - 1 = -1; 1 = p + 1
    for target in (0, V.P - 1, 1):
        reps = [l for v, l in enc if v == target]
        assert any(min(l) < 0 for l in reps) and any(max(map(abs, l)) > V.TIGHT for l in reps)      # negative and loose limbs
        assert len({V.value(l) for l in reps}) > 3                                     # several integers of the one residue
    pts = V.points(pyref)
    assert sum(p.Z != 1 for p in pts.values()) >= 8 and all(pts["d%d" % i].Z == 1 and pts["d%d" % i].X % 2 == 0 for i in range(6))
    pairs = {n: (p, q) for n, p, q in V.point_pairs(pyref)}
    assert (pairs["B+-B"][0] + pairs["B+-B"][1]) == pyref.IDENTITY and pairs["B+B"][0] is pairs["B+B"][1]
    assert all(q.Z == 1 for _, _, q in V.madd_pairs(pyref))
    names = {n for _, _, _, n in V.recode_cases()}
    assert {"blinding-allneg", "canonical-ones", "value-as-blinding-allpos", "blinding-top128"} <= names


def test_fe_mul_raw_limbs(host):
    rows = C.fe_mul(host)
    by = {}
    for (fam, _, _), h in zip(V.field_pairs(), rows):
        by.setdefault(fam, []).append(h[1])
    # the family built for it does leave limb 1 negative -- on every case, and to 85 % of the derived bound (eight of the nine
    # products of column 8 at the bound, one of them at 2/3 or more) -- and its mirror image leaves it above 2^29
    assert all(v < 0 for v in by["neglimb1"]) and min(by["neglimb1"]) <= 0.85 * V.MUL_LIMB1[0]
    assert all(v > V.M29 for v in by["poslimb1"]) and max(by["poslimb1"]) - V.M29 >= 0.85 * V.MUL_LIMB1[1]


def test_fe_sq_raw_limbs(host):
    rows = C.fe_sq(host)
    l1 = [h[1] for h in rows]
    assert min(l1) < 0 and max(l1) > V.M29                                             # both sides of [0, 2^29) are left by a square too


def test_fe_carry_addc_towords_raw_limbs(host):
    rows = C.fe_carry(host)
    l1 = [h[1] for h in rows]
    assert min(l1) == -1 and max(l1) == 2**29                                          # the carry's own excursion of limb 1: exactly one
    C.fe_addc(host)
    C.fe_towords(host)


def test_fe_abs_invert_sqrt_ratio(host, pyref):
    prods = C.fe_mul(host)
    rows = C.fe_abs(host, prods[::3])
    assert any(h[1] < 0 for h in prods[::3])                                           # inputs with a negative limb 1 went in
    assert any(V.value(f) % V.P % 2 for f in prods[::3])                               # and values that had to be negated
    C.fe_powers(host)
    C.fe_sqrt_ratio(host, pyref)
    assert rows


@pytest.mark.parametrize("op", [A.GE_MADD, A.GE_ADD, A.GE_DBL, A.GE_ADD_CACHED, A.GE_NEG, A.GE_CHAIN])
def test_group_ops_on_crafted_points(host, pyref, op):
    C.ge_op(host, pyref, op)


def test_codec_on_crafted_encodings(host, pyref):
    C.ge_codec(host, pyref)


def test_scalar_ops_on_edge_scalars(host):
    C.scalars(host)


@pytest.fixture(scope="module")
def strobe_run(host):
    return C.strobe_run(host)


@pytest.mark.parametrize("n", C.STROBE_NWORDS)
def test_transcript_replay_at_every_block_position(strobe_run, pyref, n):
    """the transcript the device tests replay in a wavefront, in the one-lane Strobe on the host: pins the expected values"""
    C.strobe_positions(strobe_run, 1)
    C.strobe_against_merlin(strobe_run, pyref, n, 1)
