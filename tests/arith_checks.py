"""The checks of the raw-limb cases, written once: each takes a Cases runner (arith_shim.py: the host path or the device path),
runs the vectors of limb_vectors.py through it, compares with big integers / pyref and with the output contract of fe.h, and
returns the raw output limbs -- the device tests then compare those with the host path's, limb for limb."""
import numpy as np

import arith_shim as A
import edge_scalars as E
import limb_vectors as V

P, L = V.P, V.L


def _limb_rows(limbs):
    return [[int(v) for v in row] for row in limbs]


def _check_point_limbs(l36, where):
    """every coordinate of a point an operation returned is a product: fe_mul's output contract"""
    for k in range(4):
        assert V.contract_ok(l36[9 * k:9 * k + 9], V.MUL_LIMB1), (where, "XYZT"[k], l36[9 * k:9 * k + 9])


def fe_mul(c):
    pairs = V.field_pairs()
    limbs, vals, _ = c.fe(A.FE_MUL, [f for _, f, _ in pairs], [g for _, _, g in pairs])
    rows = _limb_rows(limbs)
    for (fam, f, g), h, v in zip(pairs, rows, vals):
        want = V.value(f) * V.value(g) % P
        assert v == want and V.value(h) % P == want, (fam, f, g, h)
        assert V.contract_ok(h, V.MUL_LIMB1), (fam, f, g, h)
        assert h == V.model_mul(f, g), (fam, f, g, h)
    return rows


def fe_sq(c):
    ins = V.square_inputs()
    limbs, vals, _ = c.fe(A.FE_SQ, [f for _, f in ins])
    rows = _limb_rows(limbs)
    for (fam, f), h, v in zip(ins, rows, vals):
        want = V.value(f) ** 2 % P
        assert v == want and V.value(h) % P == want, (fam, f, h)
        assert V.contract_ok(h, V.SQ_LIMB1), (fam, f, h)
        assert h == V.model_sq(f), (fam, f, h)
    return rows


def fe_carry(c):
    ins = V.carry_inputs()
    limbs, vals, _ = c.fe(A.FE_CARRY, [f for _, f in ins])
    rows = _limb_rows(limbs)
    for (fam, f), h, v in zip(ins, rows, vals):
        assert v == V.value(f) % P and V.value(h) % P == v, (fam, f, h)
        assert V.contract_ok(h, V.CARRY_LIMB1), (fam, f, h)
        assert h == V.model_carry(f), (fam, f, h)
    return rows


def fe_addc(c):
    ins = V.addc_inputs()
    limbs, vals, _ = c.fe(A.FE_ADDC, [f for f, _ in ins], [g for _, g in ins])
    rows = _limb_rows(limbs)
    for (f, g), h, v in zip(ins, rows, vals):
        assert v == (V.value(f) + V.value(g)) % P and V.value(h) % P == v, (f, g, h)
        assert V.contract_ok(h, V.CARRY_LIMB1), (f, g, h)
    return rows


def fe_towords(c):
    ins = V.encoding_inputs()
    _, vals, _ = c.fe(A.FE_TOWORDS, [l for _, l in ins])
    for (v, l), got in zip(ins, vals):
        assert got == v, (v, l, got)
    return vals


def fe_abs(c, reduced_rows):
    """fe_abs on REDUCED inputs as the operations leave them (the products of fe_mul's vectors: limb 1 negative and above 2^29
    among them) and on the special values: |f| in value, and reduced again."""
    ins = reduced_rows + list(V.special_limbs().values())
    limbs, vals, _ = c.fe(A.FE_ABS, ins)
    rows = _limb_rows(limbs)
    for f, h, v in zip(ins, rows, vals):
        x = V.value(f) % P
        assert v == (P - x if x & 1 else x) and V.value(h) % P == v, (f, h)
        assert V.contract_ok(h, V.MUL_LIMB1), (f, h)                                  # f itself, or a carried -f
    return rows


def fe_powers(c):
    xs = V.field_values()
    ins = [V.limbs_of(x) for x in xs]
    inv_l, inv, _ = c.fe(A.FE_INVERT, ins)
    pw_l, pw, _ = c.fe(A.FE_POW22523, ins)
    for x, a, b in zip(xs, inv, pw):
        assert a == pow(x, P - 2, P) and b == pow(x, (P - 5) // 8, P), x
    rows = _limb_rows(inv_l) + _limb_rows(pw_l)
    assert all(V.contract_ok(h, V.MUL_LIMB1) for h in rows)
    return rows


def fe_sqrt_ratio(c, R):
    ins = V.sqrt_ratio_inputs()
    limbs, vals, flags = c.fe(A.FE_SQRT_RATIO, [V.limbs_of(u) for u, _ in ins], [V.limbs_of(v) for _, v in ins])
    seen = set()
    for (u, v), got, fl in zip(ins, vals, flags):
        ok, r = R.sqrt_ratio_m1(u, v)
        assert (bool(fl), got) == (bool(ok), r), (u, v)
        seen.add((bool(ok), u == 0))
    assert seen == {(True, True), (True, False), (False, False)}                      # zero numerator, square, non-square
    return _limb_rows(limbs)


# ------------------------------------------------------------------------------------------------ group
def _run_ge(c, R, op, triples, negs, quad=False):
    """triples: [(name, p, q)] run once per entry of negs -> (cases [(name, p, q, neg)], raw output)"""
    cases = [(n, p, q, ng) for (n, p, q) in triples for ng in negs]
    out = c.ge(op, [V.point_limbs(p) for _, p, _, _ in cases], [V.point_limbs(q) for _, _, q, _ in cases], [ng for *_, ng in cases], quad=quad)
    return cases, out


def ge_expected(R, op, p, q, neg):
    qq = -q if neg else q
    if op in (A.GE_MADD, A.GE_ADD, A.GE_ADD_CACHED):
        return p + qq
    if op == A.GE_DBL:
        return p.double()
    if op == A.GE_NEG:
        return -p
    r = p
    for _ in range(A.GE_CHAIN_ROUNDS):
        r = r + qq
        for _ in range(A.GE_CHAIN_DBLS):
            r = r.double()
    return r


def ge_cases_of(R, op):
    if op in (A.GE_MADD, A.GE_CHAIN):
        return V.madd_pairs(R), (0, 1)
    if op == A.GE_ADD:
        return V.point_pairs(R), (0,)
    if op == A.GE_ADD_CACHED:
        return V.point_pairs(R), (0, 1)
    pts = V.points(R)
    return [(n, p, p) for n, p in pts.items()], (0,)                                  # GE_DBL, GE_NEG


def ge_op(c, R, op):
    """one per-lane group operation on its points: encoding against pyref, every output coordinate within the contract"""
    triples, negs = ge_cases_of(R, op)
    cases, (limbs, encs) = _run_ge(c, R, op, triples, negs)
    rows = _limb_rows(limbs)
    for (name, p, q, ng), l36, enc in zip(cases, rows, encs):
        want = ge_expected(R, op, p, q, ng)
        assert enc == want.compress(), (op, name, ng)
        assert V.point_of_limbs(R, l36) == want, (op, name, ng)
        if op != A.GE_NEG:
            _check_point_limbs(l36, (op, name, ng))
    return rows


def ge_codec(c, R):
    encs = V.encodings(R)
    ok, limbs, again = c.decompress(encs)
    n_ok = 0
    for e, o, l36, a in zip(encs, ok, _limb_rows(limbs), again):
        ref = R.decompress(e)
        assert bool(o) == (ref is not None), e.hex()
        if ref is not None:
            n_ok += 1
            assert a == e and V.value(l36[:9]) % P == ref.X and V.value(l36[9:18]) % P == ref.Y, e.hex()
            assert ref.X % 2 == 0                                                     # |x| returned
    assert 10 < n_ok < len(encs) - 10                                                 # valid and invalid both
    us = V.uniform_inputs()
    ul, uenc = c.uniform(us)
    for u, l36, e in zip(us, _limb_rows(ul), uenc):
        assert e == R.from_uniform_bytes(u).compress(), u.hex()
        _check_point_limbs(l36, "from_uniform")
    return _limb_rows(limbs), _limb_rows(ul)


# ------------------------------------------------------------------------------------------------ scalars
def scalars(c):
    pairs = V.scalar_pairs()
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    out = {}
    for op, f in ((A.SC_MUL, lambda x, y: x * y % L), (A.SC_ADD, lambda x, y: (x + y) % L), (A.SC_SUB, lambda x, y: (x - y) % L),
                  (A.SC_MONTMUL_RAW, lambda x, y: x * y * pow(2**256, -1, L) % L)):
        out[op] = c.sc(op, a, b)
        assert out[op] == [f(x, y) for x, y in pairs], op
    few = [x for x in a[:40]]                                                          # the edge pairs among them; 0 -> 0
    for op in (A.SC_INVERT, A.SC_INVERT_VARTIME):
        out[op] = c.sc(op, few, [0] * len(few))
        assert out[op] == [pow(x % L, L - 2, L) for x in few], op
    u = [0, 1, 2**32 - 1, 2**32, 2**64 - 1, 2**63] + [x % 2**64 for x in a[14:40]]
    out[A.SC_FROM_U64] = c.sc(A.SC_FROM_U64, u, [0] * len(u))
    assert out[A.SC_FROM_U64] == u
    ws = V.wide_inputs()
    out["wide"] = c.sc_wide(ws)
    assert out["wide"] == [int.from_bytes(w, "little") % L for w in ws]
    rc = V.recode_cases()
    out["recode"] = c.recode(rc)
    hit_neg = 0
    for (W, NW, x, name), d in zip(rc, out["recode"]):
        assert d == E.recode(x, W, NW), (W, NW, name)
        assert sum(v << (W * i) for i, v in enumerate(d)) == x and all(abs(v) <= 1 << (W - 1) for v in d), (W, NW, name)
        hit_neg += d.count(-(1 << (W - 1)))
    assert hit_neg > 10 * len(E.WIDTHS)                                               # the row-end digit -2^(W-1) is reached at every width
    return out


# ------------------------------------------------------------------------------------------------ STROBE / Merlin
STROBE_NWORDS = (1, 2, 8, 16, 50)                     # message words: 50 words = 200 bytes span more than one 166-byte block


def strobe_run(c):
    """one call for every (filler length k, message words n): k = 0..165 puts the first message word at every block position"""
    rng = np.random.default_rng(47)
    filler = bytes(rng.integers(0, 256, size=166, dtype=np.uint8))
    words = rng.integers(0, 2**32, size=max(STROBE_NWORDS), dtype=np.uint32)
    kn = [(k, n) for n in STROBE_NWORDS for k in range(166)]
    out, pos = c.strobe(kn, filler, words, words[::-1].copy())
    return kn, filler, words, out, pos


def strobe_positions(run, holder):
    kn, _, _, _, pos = run
    for n in STROBE_NWORDS:
        at = sorted(int(pos[i][holder]) for i, (k, nn) in enumerate(kn) if nn == n)
        assert at == list(range(166))                 # the first message word at EVERY offset: 162 ends on the block, 163..165 cross it


def strobe_against_merlin(run, R, n, holder):
    """both challenges of the replayed transcript against pyref.Transcript, for every block position of the first word"""
    kn, filler, words, out, pos = run
    msg = words[:n].astype("<u4").tobytes()
    rev = words[::-1][:n].astype("<u4").tobytes()
    head = R.Transcript(b"dev-shim")
    for i, (k, nn) in enumerate(kn):
        if nn != n:
            continue
        t = head.clone()
        t.append_message(b"fill", filler[:k])
        t.append_message(b"words", msg)
        c1 = t.challenge_bytes(b"c1", 64)
        t.append_message(b"more", rev)
        c2 = t.challenge_bytes(b"c2", 64)
        assert out[i][holder].astype("<u4").tobytes() == c1 + c2, (k, n, int(pos[i][holder]))
